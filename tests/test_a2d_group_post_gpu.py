"""GPU: the A2D-Sentences / JHMDB-Sentences output stage for a group of samples (include/tce_rvos_eval.h, ops.a2d_group_masks,
A2DSentencesPostProcess(grouped=True)) against the per-sample launches it replaces: every byte ops.a2d_masks', every score
ops.sigmoid's, sample 0 of the first case against the reference class's fixture (tests/golden/a2d_post_cases.npz), and the
entry's access model against the bytes the launch touches (tests/_footprint.py)."""
import os

import pytest
import torch

import _a2d
import _footprint as fp
from tce_rvos_amd import _lib, hazard

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "a2d_post_cases.npz")


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in _a2d.load_cases(FIXTURE)}


@pytest.fixture(scope="module")
def three(cases):
    """B = 3 on N = 5 planes of 18 x 25: case A's own (size, orig), an output of one pixel, an up-scale to odd extents.  Inputs, the
    per-sample launches' results (the reference of every test here; computed once, never modified) and the group launch's."""
    from tce_rvos_amd import ops
    a = cases["A"]
    pairs = [(a["size"], a["orig"]), ((72, 100), (1, 1)), ((50, 97), (211, 173))]
    pm = [a["masks"].cuda()] + [_a2d.make_inputs(50 + i, 5, (18, 25), "smooth", 6.0)[1].cuda() for i in (1, 2)]
    lg = [a["logits"].cuda()] + [_a2d.make_inputs(50 + i, 5, (18, 25), "smooth", 6.0)[0].cuda() for i in (1, 2)]
    solo_m = [ops.a2d_masks(m, s, o) for m, (s, o) in zip(pm, pairs)]
    solo_s = [ops.sigmoid(l) for l in lg]
    masks, scores = ops.a2d_group_masks(pm, lg, [p[0] for p in pairs], [p[1] for p in pairs])
    torch.cuda.synchronize()
    return dict(pm=pm, lg=lg, pairs=pairs, solo_m=solo_m, solo_s=solo_s, masks=masks, scores=scores)


def test_group_launch_equals_the_per_sample_launches(three, cases):
    t = three
    assert len(t["masks"]) == len(t["scores"]) == 3
    for b in range(3):
        H0, W0 = t["pairs"][b][1]
        assert t["masks"][b].dtype == torch.uint8 and tuple(t["masks"][b].shape) == (5, H0, W0)
        assert torch.equal(t["masks"][b], t["solo_m"][b]), b
        assert t["scores"][b].dtype == torch.float32 and tuple(t["scores"][b].shape) == (5,)
        assert torch.equal(t["scores"][b], t["solo_s"][b]), b
    a = cases["A"]
    _a2d.check_masks(t["masks"][0], a["ref"], a["contested"], "case A through the group launch")
    assert int(t["masks"][2].sum()) > 0 and int((t["masks"][2] == 0).sum()) > 0  # the up-scaled sample is no constant plane


def test_outputs_at_odd_addresses_leave_the_guard_bytes_alone(three):
    from tce_rvos_amd import ops
    t = three
    sizes = [m.numel() for m in t["solo_m"]]
    offs, at = [], 1
    for b, n in enumerate(sizes):   # sample b starts at an odd address (1, 3 and 1 mod 4 here), 5 or 6 guard bytes behind each
        offs.append(at)
        at += n + 5
        at += 1 - at % 2
    flat = torch.full((at + 7,), 0xEE, dtype=torch.uint8, device="cuda")
    outs = [flat[o:o + n].view(*m.shape) for o, n, m in zip(offs, sizes, t["solo_m"])]
    assert all(o.data_ptr() % 2 == 1 for o in outs) and len({o.data_ptr() % 4 for o in outs}) == 2
    masks, scores = ops.a2d_group_masks(t["pm"], t["lg"], [p[0] for p in t["pairs"]], [p[1] for p in t["pairs"]], outs=outs)
    torch.cuda.synchronize()
    guard = torch.ones_like(flat, dtype=torch.bool)
    for b in range(3):
        assert masks[b].data_ptr() == outs[b].data_ptr() and torch.equal(outs[b], t["solo_m"][b]), b
        assert torch.equal(scores[b], t["solo_s"][b])
        guard[offs[b]:offs[b] + sizes[b]] = False
    assert int(guard.sum()) >= 1 + 5 + 5 + 7 and bool((flat[guard] == 0xEE).all())


def test_one_more_sample_than_a_launch_table_holds(cases):
    from tce_rvos_amd import ops
    d = cases["D"]
    B = ops.A2D_GROUP_MAX + 1
    pm = [_a2d.make_inputs(200 + b, 2, (3, 4), "noise", 1.0)[1].cuda() for b in range(B)]
    lg = [_a2d.make_inputs(200 + b, 2, (3, 4), "noise", 1.0)[0].cuda() for b in range(B)]
    pm[0], lg[0] = d["masks"].cuda(), d["logits"].cuda()
    origs = [d["orig"]] + [(5 + b % 3, 7 + b % 4) for b in range(1, B)]
    masks, scores = ops.a2d_group_masks(pm, lg, [d["size"]] * B, origs)
    torch.cuda.synchronize()
    assert len(masks) == len(scores) == B
    for b in range(B):
        assert torch.equal(masks[b], ops.a2d_masks(pm[b], d["size"], origs[b])), b
        assert torch.equal(scores[b], ops.sigmoid(lg[b])), b
    _a2d.check_masks(masks[0], d["ref"], d["contested"], "case D through the group launch")


def test_strided_logit_views_are_read_in_place(three):
    """pred_logits [B,T,N,K] with K > 1: the class column is a strided view; the launch reads it where it is."""
    from tce_rvos_amd import ops
    t = three
    wide = [torch.stack([l, l + 1.0, l - 2.0], 1) for l in t["lg"]]   # [N, 3]
    _, scores = ops.a2d_group_masks(t["pm"], [w[:, 0] for w in wide], [p[0] for p in t["pairs"]], [p[1] for p in t["pairs"]])
    torch.cuda.synchronize()
    for b in range(3):
        assert torch.equal(scores[b], t["solo_s"][b]), b


@pytest.mark.parametrize("rle", [True, False])
def test_grouped_post_processor_equals_the_per_sample_one(three, rle):
    from tce_rvos_amd.postprocess import A2DSentencesPostProcess
    t = three
    outs = [{"pred_logits": l.view(1, 1, -1, 1), "pred_masks": m[None, None]} for l, m in zip(t["lg"], t["pm"])]
    # a sample of another plane in the middle: it goes through a group launch of its own, the order of the results is the input's
    g = torch.Generator().manual_seed(9)
    outs.insert(1, {"pred_logits": torch.randn(1, 1, 5, 1, generator=g).cuda(), "pred_masks": (torch.randn(1, 1, 5, 9, 11, generator=g) * 3).cuda()})
    orig = [t["pairs"][0][1], (30, 41), t["pairs"][1][1], t["pairs"][2][1]]
    size = [t["pairs"][0][0], (36, 44), t["pairs"][1][0], t["pairs"][2][0]]
    want = A2DSentencesPostProcess(rle=rle)(outs, orig, size)
    got = A2DSentencesPostProcess(rle=rle, grouped=True)(outs, orig, size)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 4
    for r, w in zip(got, want):
        assert set(r) == set(w) == ({"scores", "masks", "rle_masks"} if rle else {"scores", "masks"})
        assert torch.equal(r["scores"], w["scores"]) and torch.equal(r["masks"], w["masks"]) and r["masks"].shape == w["masks"].shape
        if rle:
            assert r["rle_masks"] == w["rle_masks"]
    for b, k in ((0, 0), (2, 1), (3, 2)):
        assert torch.equal(got[b]["masks"][:, 0], t["solo_m"][k])


# --------------------------------------------------------------------------------------------- the recorder and the footprint
def test_hazard_recording_lists_the_one_entry(three):
    from tce_rvos_amd import ops
    t = three
    with hazard.recording() as rec:
        masks, scores = ops.a2d_group_masks(t["pm"], t["lg"], [p[0] for p in t["pairs"]], [p[1] for p in t["pairs"]])
    torch.cuda.synchronize()
    assert [x.name for x in rec.launches] == ["tce_a2d_group_masks_u8"] and rec.analyse().clean
    for b in range(3):
        assert torch.equal(masks[b], t["masks"][b]) and torch.equal(scores[b], t["scores"][b]), b


@pytest.fixture(scope="module")
def slab():
    s = fp.Slab(64 << 20, device="cuda")
    yield s
    del s
    torch.cuda.empty_cache()


def _group_case(S, N, h, w, samples):
    """samples: per sample (fh, fw, H0, W0, the bytes `out` starts into its buffer, logit_stride).  Every device buffer of the call in
    the slab: the mask planes and the scores of all samples in one buffer each, logits and out per sample.  The table is a host
    array, read by the entry point at the call: it stays outside the slab."""
    B = len(samples)
    pm = S.randn("masks", (B, N * h * w), scale=3.0)
    scores = S.alloc("scores", (B, N))
    table = (_lib.A2dGroupSample * B)()
    lg, raws = [], []
    for b, (fh, fw, H0, W0, shift, stride) in enumerate(samples):
        lg.append(S.randn(f"logits{b}", (N * stride,), scale=2.0))
        raws.append(S.alloc(f"out{b}", (shift + N * H0 * W0 + 3,), dtype=torch.uint8))
        e = table[b]
        e.masks, e.logits, e.out, e.scores = pm[b].data_ptr(), lg[b].data_ptr(), raws[b].data_ptr() + shift, scores[b].data_ptr()
        e.fh, e.fw, e.H0, e.W0, e.logit_stride = fh, fw, H0, W0, stride

    def fn():
        _lib.check(_lib.lib().tce_a2d_group_masks_u8(table, B, N, h, w, 0.5, torch.cuda.current_stream().cuda_stream),
                   "tce_a2d_group_masks_u8")
    fn.check = lambda: (pm, lg, raws, scores)
    return fn


GROUP_FOOTPRINT = [
    # the second sample's planes of 20 x 30 x 3 = 1800 bytes take more than one 1024-byte workgroup; its logits are 2 floats apart
    ("two_samples_3x4x6_to_9x11_and_20x30_addresses_1_and_2", dict(N=3, h=4, w=6, samples=[(13, 20, 9, 11, 1, 1), (16, 24, 20, 30, 2, 2)])),
    ("a_full_table_of_16_samples_1x2x2_to_3x5", dict(N=1, h=2, w=2, samples=[(7, 8, 3, 5, b % 4, 1) for b in range(16)])),
]


@pytest.mark.parametrize("tag,kw", GROUP_FOOTPRINT, ids=[c[0] for c in GROUP_FOOTPRINT])
def test_a2d_group_masks_footprint(slab, tag, kw):
    """W, O and R of tests/_footprint.py, no exemptions: nothing outside the samples' out and scores is written (the bytes around the
    oddly placed planes included), every output byte and every score is written, and the result depends on no byte outside the
    samples' mask planes and the N logits of each -- the floats between strided logits included."""
    from tce_rvos_amd import ops
    info = fp.check_case(slab, lambda S: _group_case(S, **kw), fp.recorder("tce_a2d_group_masks_u8"), props="WOR",
                         sync=torch.cuda.synchronize, label=tag)
    print(f"{tag}: read {info['read_bytes']} written {info['written_bytes']} guard {info['guard_bytes']} untouched-in-buffers {info['pad_bytes']}")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == []
    N, h, w, samples = kw["N"], kw["h"], kw["w"], kw["samples"]
    assert info["read_bytes"] == len(samples) * (N * h * w + N) * 4
    assert info["written_bytes"] == sum(N * s[2] * s[3] + N * 4 for s in samples)
    slab.begin(0)
    fn = _group_case(slab, **kw)
    fn()
    pm, lg, raws, scores = fn.check()
    for b, (fh, fw, H0, W0, shift, stride) in enumerate(samples):
        want = ops.a2d_masks(pm[b].reshape(N, h, w).clone(), (fh, fw), (H0, W0))
        assert torch.equal(raws[b][shift:shift + N * H0 * W0], want.reshape(-1)), b
        assert torch.equal(scores[b], ops.sigmoid(lg[b][::stride].clone())), b


def test_rejections():
    from tce_rvos_amd import ops
    pm = torch.zeros(2, 4, 6, device="cuda")
    lg = torch.zeros(2, device="cuda")
    with pytest.raises(ValueError, match="at least one"):
        ops.a2d_group_masks([], [], [], [])
    with pytest.raises(ValueError, match="contiguous"):
        ops.a2d_group_masks([pm, torch.zeros(2, 4, 12, device="cuda")[..., ::2]], [lg, lg], [(16, 24)] * 2, [(8, 10)] * 2)
    with pytest.raises(ValueError, match="on the GPU"):
        ops.a2d_group_masks([pm.cpu()], [lg.cpu()], [(16, 24)], [(8, 10)])
    with pytest.raises(ValueError, match="4x"):
        ops.a2d_group_masks([pm, pm], [lg, lg], [(16, 24), (17, 24)], [(8, 10)] * 2)
    with pytest.raises(ValueError, match="4x"):
        ops.a2d_group_masks([pm], [lg], [(16, 25)], [(8, 10)])
    with pytest.raises(ValueError, match="2\\^31"):
        ops.a2d_group_masks([pm], [lg], [(16, 24)], [(40000, 40000)])
    with pytest.raises(ValueError, match="sample 1"):
        ops.a2d_group_masks([pm, torch.zeros(2, 4, 7, device="cuda")], [lg, lg], [(16, 24)] * 2, [(8, 10)] * 2)
    with pytest.raises(ValueError, match="logits"):
        ops.a2d_group_masks([pm], [torch.zeros(3, device="cuda")], [(16, 24)], [(8, 10)])
    with pytest.raises(ValueError):
        ops.a2d_group_masks([pm, pm], [lg, lg], [(16, 24)], [(8, 10)] * 2)
    with pytest.raises(ValueError):
        ops.a2d_group_masks([pm], [lg], [(16, 24)], [(8, 10)], outs=[torch.empty(2, 8, 11, dtype=torch.uint8, device="cuda")])
    masks, scores = ops.a2d_group_masks([pm], [lg], [(16, 24)], [(8, 10)])  # all-zero logits: sigmoid 0.5 is not above 0.5
    torch.cuda.synchronize()
    assert not bool(masks[0].any()) and bool((scores[0] == 0.5).all())
